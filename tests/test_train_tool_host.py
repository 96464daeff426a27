"""The host side of tools/train.py: the arguments, tables / samplers / plan from annotation files, the validation directory.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from pairdata import tiny_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("train_tool", os.path.join(ROOT, "tools", "train.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


def test_arguments_and_their_defaults(tmp_path):
    args = tool.parse_args(["--data", "a.csv", "/data/a"])
    assert args.data == [["a.csv", "/data/a"]]
    assert (args.negative_ratio, args.frame_offset, args.clip_range, args.num_samples, args.bn_momentum) == (0.0, 70, False, 100000, 0.1)
    assert (args.optimizer, args.lr, args.epochs, args.batch, args.scale, args.prefetch, args.val_dir) == ("adam", 1e-4, 50, 128, 1, 1, None)
    assert tool.frame_offsets(args) is None
    args = tool.parse_args("--data a.csv /a --data b.csv /b --clip-range --dynamic-frame-offset 20 5 5 150 --optimizer sgd --scale 2 "
                           "--val-dir v --batch 4 --epochs 3".split())
    assert args.data == [["a.csv", "/a"], ["b.csv", "/b"]] and args.clip_range and args.optimizer == "sgd" and args.scale == 2
    assert tool.frame_offsets(args) == dict(start_epoch=20, freq=5, step=5, max_value=150)
    for bad in (["--epochs", "3"], ["--data", "a.csv"], ["--data", "a.csv", "/a", "--scale", "3"], ["--data", "a.csv", "/a", "--optimizer", "lamb"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_tables_samplers_and_plan_from_annotation_files(tmp_path):
    first, second = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    tiny_table().to_csv(first)
    tiny_table(datasets=("coco", "coco", "coco")).to_csv(second)
    args = tool.parse_args(["--data", first, "/data/a", "--data", second, "/data/b", "--num-samples", "10", "--frame-offset", "2", "--clip-range",
                            "--negative-ratio", "1", "--batch", "4", "--seed", "3"])
    tables, samplers, plan = tool.make_plan(args)
    assert [t.root for t in tables] == ["/data/a", "/data/b"] and [len(t) for t in tables] == [15, 15]
    assert tables[1].paths()[0] == "/data/b/a/0000.jpg" and set(tables[1].dataset.tolist()) == {"coco"}
    assert all(len(s) == 10 and s.frame_offset == 2 and s.clip_range and s.rows.size == 15 for s in samplers)
    assert not np.array_equal(samplers[0].epoch_rows, samplers[1].epoch_rows)          # each its own seed
    assert plan.samplers == samplers and len(plan) == 5 and plan.start_epoch().shape == (5, 4)
    again = tool.make_plan(args)[2]
    assert np.array_equal(again.start_epoch(), plan.batches)                           # the seed decides


class Store:
    """What `read_sequences` and `StoreFrames` use of a JpegStore."""

    def __init__(self):
        self.files = []

    def add(self, items):
        self.files += list(items)
        return np.arange(len(self.files) - len(items), len(self.files), dtype=np.int64)

    def _checked(self, ids):
        return np.asarray(ids, dtype=np.int64).reshape(-1)


def test_validation_directory(tmp_path):
    for name, frames, boxes in (("s1", 4, 4), ("s2", 3, 5), ("empty", 0, 2), ("untracked", 3, 0)):
        os.makedirs(tmp_path / name)
        for k in range(frames):
            (tmp_path / name / f"{k:08d}.jpg").write_bytes(b"x")
        if boxes:
            (tmp_path / name / "groundtruth.txt").write_text("".join(f"{10 + k}.5,20,30,40\n" for k in range(boxes)))
    store = Store()
    seqs = tool.read_sequences(str(tmp_path), store, "val", chunk=3)
    assert [(len(f), b.shape, n) for f, b, n in seqs] == [(4, (4, 4), "val"), (3, (3, 4), "val")]
    assert seqs[0][1][1].tolist() == [11.5, 20, 30, 40] and seqs[1][0].ids.tolist() == [4, 5, 6]
    assert [os.path.basename(p) for p in store.files[:4]] == [f"{k:08d}.jpg" for k in range(4)]
    with pytest.raises(SystemExit):
        tool.read_sequences(str(tmp_path / "empty"), store, "val")
