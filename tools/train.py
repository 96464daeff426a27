"""Train FEAR-XS from annotation tables: the counterpart of the reference's `train.py` over `feartracker_amd.fit`.

    python tools/train.py --data got10k/train.csv /data/fear/got10k --num-samples 100000 --frame-offset 70 --clip-range \\
        --dynamic-frame-offset 20 5 5 150 --optimizer adam --lr 1e-4 --epochs 50 --batch 128 --val-dir /data/fear/got10k/val --out runs/xs

--data CSV ROOT     an annotation file of the reference's (track_id, frame_index, img_path, bbox, presence, near_corner, dataset) and the
                    directory its img_path values are relative to; repeat it for several datasets (the reference's ConcatDataset)
sampler keys        --negative-ratio, --frame-offset, --clip-range, --num-samples, --dynamic-frame-offset START FREQ STEP MAX: the keys of
                    config/dataset/*.yaml, applied to every --data
--val-dir DIR       every sub-directory is a sequence: its *.jpg files in name order and groundtruth.txt with one "x,y,w,h" per line
                    (GOT-10k's layout); validated every --val-every epochs under the dataset name --val-name
--scale 2|4|8       decode the training frames at that fraction (JpegStore.decode_rows(scale=))
--scale auto        per batch and frame the largest fraction that upsamples no crop read from the frame (TrainPairBuilder.frame_scales),
                    at most 1 / --max-scale
--windows           decode per frame only the rectangle a batch reads, as compact frames (JpegStore.decode_windows)
--store-residence host   keep the files' scan bytes in pinned host memory (JpegStore(residence="host")): the device holds the indexes and
                    tables alone, about a ninth of a file's footprint, and --host-capacity-gb limits the pinned bytes
Every file is decoded from a JpegStore, so the datasets must fit in --capacity-gb of device memory (with --store-residence host: their
indexes there and their bytes in --host-capacity-gb of pinned host memory).  The run writes last.pt (resumed
from with --resume), the best three .fearw files and history.json under --out.  After every epoch the tool calls `store.check()`: the
store keeps the statuses of its last `JpegStore.PENDING_CALLS` (64) decode calls only, so that is a check of the epoch's last batches
and of the validation's decodes, not of every batch (the files themselves were judged in full when they were added)."""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_sequences(directory, store, name, chunk=4096):
    """[(StoreFrames, (T, 4) boxes, name)] for the sequences under `directory`, their frames added to `store`."""
    from feartracker_amd import StoreFrames
    out = []
    for seq in sorted(glob.glob(os.path.join(directory, "*", ""))):
        truth = os.path.join(seq, "groundtruth.txt")
        files = sorted(glob.glob(os.path.join(seq, "*.jpg")))
        if not os.path.exists(truth) or len(files) < 2:
            continue
        boxes = np.loadtxt(truth, delimiter=",", ndmin=2)[:, :4]
        n = min(len(files), len(boxes))
        ids = np.concatenate([store.add(files[at:at + chunk]) for at in range(0, n, chunk)])
        out.append((StoreFrames(store, ids), boxes[:n], name))
    if not out:
        raise SystemExit(f"{directory}: no sequence with *.jpg frames and groundtruth.txt")
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", nargs=2, action="append", required=True, metavar=("CSV", "ROOT"))
    ap.add_argument("--negative-ratio", type=float, default=0.0)
    ap.add_argument("--frame-offset", type=int, default=70)
    ap.add_argument("--clip-range", action="store_true")
    ap.add_argument("--num-samples", type=int, default=100000)
    ap.add_argument("--dynamic-frame-offset", type=int, nargs=4, default=None, metavar=("START", "FREQ", "STEP", "MAX"))
    ap.add_argument("--optimizer", default="adam", choices=("adam", "adamw", "sgd"))
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--gradient-clip", type=float, default=0.0)
    ap.add_argument("--bn-momentum", type=float, default=0.1, help="momentum of the BatchNorm running statistics")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--min-epochs", type=int, default=0)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--scale", type=lambda v: v if v == "auto" else int(v), default=1, choices=(1, 2, 4, 8, "auto"))
    ap.add_argument("--max-scale", type=int, default=8, choices=(1, 2, 4, 8), help="the largest scale --scale auto picks")
    ap.add_argument("--windows", action="store_true", help="decode the rectangles a batch reads as compact frames")
    ap.add_argument("--photometric", action="store_true", help="the photometric stage of the data builder")
    ap.add_argument("--prefetch", type=int, default=1, choices=(0, 1))
    ap.add_argument("--val-dir", default=None)
    ap.add_argument("--val-name", default="val")
    ap.add_argument("--val-every", type=int, default=1)
    ap.add_argument("--max-val-samples", type=int, default=200)
    ap.add_argument("--early-stopping", type=int, default=20)
    ap.add_argument("--capacity-gb", type=float, default=None)
    ap.add_argument("--store-residence", default="device", choices=("device", "host"), help="where the store keeps the files' scan bytes")
    ap.add_argument("--host-capacity-gb", type=float, default=None, help="with --store-residence host: the limit of the pinned host bytes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--out", default="runs/fear_xs")
    return ap.parse_args(argv)


def make_plan(args):
    """(tables, samplers, plan) from the arguments: host work only, no GPU."""
    from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler, TrackTable
    tables = [TrackTable.from_csv(path, root=root) for path, root in args.data]
    samplers = [TrackSampler(t, args.negative_ratio, args.frame_offset, args.num_samples, clip_range=args.clip_range, seed=args.seed + 1 + k)
                for k, t in enumerate(tables)]
    return tables, samplers, EpochPlan(samplers, args.batch, seed=args.seed)


def frame_offsets(args):
    """--dynamic-frame-offset as `EpochPlan.end_epoch` takes it, or None."""
    if not args.dynamic_frame_offset:
        return None
    return dict(zip(("start_epoch", "freq", "step", "max_value"), args.dynamic_frame_offset))


def main(argv=None):
    args = parse_args(argv)
    from feartracker_amd import JpegStore
    from feartracker_amd.fit import fit
    from feartracker_amd.metrics import TrainMetrics
    from feartracker_amd.optim import make_optimizer
    from feartracker_amd.schedule import EarlyStopping, PlateauSchedule, TopKCheckpoints
    from feartracker_amd.train_data import TrainPairBuilder
    from feartracker_amd.train_data.loader import PairLoader, fill_store
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    from feartracker_amd.validate import SequenceValidator

    os.makedirs(args.out, exist_ok=True)
    tables, samplers, plan = make_plan(args)
    if args.host_capacity_gb is not None and args.store_residence != "host":
        raise SystemExit("--host-capacity-gb goes with --store-residence host")
    store = JpegStore(device=args.device, capacity_bytes=None if args.capacity_gb is None else int(args.capacity_gb * 2 ** 30),
                      residence=args.store_residence,
                      host_capacity_bytes=None if args.host_capacity_gb is None else int(args.host_capacity_gb * 2 ** 30))
    row_ids = fill_store(store, tables)
    print(f"{sum(map(len, tables))} rows, {len(store)} files, {store.nbytes / 2 ** 20:.0f} MiB resident on the device, "
          f"{store.host_nbytes / 2 ** 20:.0f} MiB in pinned host memory")
    builder = TrainPairBuilder(dict(photometric=True) if args.photometric else None, device=args.device, seed=args.seed)
    loader = PairLoader(plan, store, row_ids, builder, scale=args.scale, prefetch=args.prefetch, windows=args.windows,
                        max_scale=args.max_scale)
    net = FEARNetTrainHIP(random_init_state(args.seed), device=args.device, momentum=args.bn_momentum)
    cfg = {"name": args.optimizer, "lr": args.lr}
    opt = make_optimizer(net, cfg, gradient_clip_val=args.gradient_clip)
    sequences = read_sequences(args.val_dir, store, args.val_name) if args.val_dir else None
    offsets = frame_offsets(args)

    class Validator:                     # a fresh engine on the epoch's weights, the reference's max_val_samples
        def run(self, seqs):
            return SequenceValidator.from_training_state(net.state_dict(), device=args.device, max_samples=args.max_val_samples).run(seqs)

    def log(record):
        print(json.dumps(record))
        store.check()

    last = os.path.join(args.out, "last.pt")
    history = fit(net, opt, loader, epochs=args.epochs, min_epochs=args.min_epochs, metrics=TrainMetrics(args.device, loader.datasets),
                  validator=Validator() if sequences else None, val_sequences=sequences, schedule=PlateauSchedule(opt),
                  checkpoints=TopKCheckpoints(os.path.join(args.out, "checkpoints")), early_stopping=EarlyStopping(args.early_stopping),
                  check_val_every_n_epoch=args.val_every, dynamic_frame_offset=offsets, resume=args.resume, checkpoint_path=last, log=log)
    with open(os.path.join(args.out, "history.json"), "w") as fh:
        json.dump(history, fh, indent=1)


if __name__ == "__main__":
    main()
