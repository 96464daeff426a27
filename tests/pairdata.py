"""The tiny dataset of the sampler, loader and fit tests: 3 tracks x 5 frames in two frame sizes, one `presence == 0` row, one
`near_corner` row, boxes that overhang their frames; its frames as 4:2:0 JPEG files written by `jpeg_encode_host`."""
import os

import numpy as np

from feartracker_amd.train_data.sampling import TrackTable

SIZES = {"a": (64, 96), "b": (72, 80), "c": (64, 96)}            # (H, W) per track
FRAMES = 5


def tiny_table(root=None, datasets=("got10k", "lasot", "got10k")) -> TrackTable:
    rng = np.random.default_rng(5)
    cols = dict(track_id=[], frame_index=[], img_path=[], bbox=[], presence=[], near_corner=[], dataset=[])
    for (track, (H, W)), dataset in zip(SIZES.items(), datasets):
        for t in range(FRAMES):
            w, h = int(rng.integers(14, 30)), int(rng.integers(12, 26))
            x, y = int(rng.integers(-4, W - w + 4)), int(rng.integers(-4, H - h + 4))
            cols["track_id"].append(track)
            cols["frame_index"].append(t)
            cols["img_path"].append(f"{track}/{t:04d}.jpg")
            cols["bbox"].append([x + 0.5 * (t == 1), y, w, h])
            cols["presence"].append(0 if (track, t) == ("b", 2) else 1)
            cols["near_corner"].append((track, t) == ("c", 3))
            cols["dataset"].append(dataset)
    return TrackTable.from_arrays(root=root, **cols)


def frame_pixels(track: str, t: int) -> np.ndarray:
    """A smooth uint8 (H, W, 3) picture with a brighter blob that moves with t, different per track."""
    H, W = SIZES[track]
    k = "abc".index(track)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 110 + 60 * np.sin(x / (9.0 + k) + t) * np.cos(y / (7.0 + 2 * k) - 0.5 * t)
    blob = 90 * np.exp(-(((x - W / 2 - 4 * t) / 12.0) ** 2 + ((y - H / 2 + 2 * t) / 9.0) ** 2))
    img = np.stack([base + blob, base * 0.8 + 30 + blob * 0.5, 200 - base * 0.6 + 10 * k], axis=-1)
    return np.clip(img, 0, 255).astype(np.uint8)


def write_frames(root: str, table: TrackTable, quality: int = 90) -> None:
    from feartracker_amd.jpeg_encode import jpeg_encode_host
    done = set()
    for path, track, t in zip(table.img_path.tolist(), table.track_id.tolist(), table.frame_index.tolist()):
        if path in done:
            continue
        done.add(path)
        full = os.path.join(root, path)
        os.makedirs(os.path.dirname(full), exist_ok=True)
        with open(full, "wb") as fh:
            fh.write(jpeg_encode_host(frame_pixels(track, int(t)), quality=quality, subsampling="4:2:0"))
