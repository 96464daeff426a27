"""The host side of training from annotation tables (feartracker_amd/train_data/sampling.py, loader.clip_boxes): the CSV reader and
its hand parser, the sampler's rules as distributions, the epoch plan, the states.  No GPU."""
import numpy as np
import pytest

from feartracker_amd.geometry import ensure_bbox_boundaries
from feartracker_amd.train_data.loader import clip_boxes
from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler, TrackTable, kept_negatives, parse_bbox, update_offset
from pairdata import tiny_table


def big_table(tracks=6, per_track=40, negatives_every=5, seed=3):
    """`tracks` tracks with unsorted frame indices (one repeated), every `negatives_every`-th row negative, some near_corner."""
    rng = np.random.default_rng(seed)
    cols = dict(track_id=[], frame_index=[], img_path=[], bbox=[], presence=[], near_corner=[], dataset=[])
    for t in range(tracks):
        frames = rng.permutation(per_track) * 3
        frames[1] = frames[0]                                            # two rows of one frame
        for k, f in enumerate(frames):
            cols["track_id"].append(f"t{t}")
            cols["frame_index"].append(int(f))
            cols["img_path"].append(f"t{t}/{k}.jpg")
            cols["bbox"].append([1, 2, 30, 40])
            cols["presence"].append(0 if k % negatives_every == 2 else 1)
            cols["near_corner"].append(k % 7 == 3)
            cols["dataset"].append("d")
    order = rng.permutation(len(cols["track_id"]))                       # tracks interleaved in the file
    return TrackTable.from_arrays(**{name: [v[i] for i in order] for name, v in cols.items()})


# ----------------------------------------------------------------------------------------------------------------------------- CSV
def test_parse_bbox_by_hand():
    assert parse_bbox("[1, 2, 3, 4]") == [1.0, 2.0, 3.0, 4.0]
    assert parse_bbox(" [ -1.5,2.25 , 3e1, +4.0] ") == [-1.5, 2.25, 30.0, 4.0]
    assert parse_bbox("(0, -7, 12, 5)") == [0.0, -7.0, 12.0, 5.0]
    for bad in ("1, 2, 3, 4", "[1, 2, 3]", "[1, 2, 3, 4, 5]", "[1, 2, 3, x]", "[1, 2, 3, __import__('os')]", "[1, 2, 3, 4", "", "[nan, 0, 1, 1]",
                "[1, 2, 3, 2*2]"):
        with pytest.raises(ValueError):
            parse_bbox(bad)


def test_csv_round_trip_and_errors(tmp_path):
    table = tiny_table(root="/data")
    path = str(tmp_path / "anno.csv")
    table.to_csv(path)
    back = TrackTable.from_csv(path, root="/data")
    for name in ("track_id", "frame_index", "img_path", "bbox", "presence", "near_corner", "dataset"):
        assert np.array_equal(getattr(back, name), getattr(table, name)), name
    assert back.bbox.dtype == np.float64 and (back.bbox % 1 != 0).any() and (back.bbox < 0).any()
    assert back.paths()[0] == "/data/a/0000.jpg" and TrackTable.from_csv(path).paths()[0] == "a/0000.jpg"
    assert list(back.track_rows) == ["a", "b", "c"]
    assert all(np.array_equal(back.track_rows[t], np.arange(5) + 5 * k) for k, t in enumerate("abc"))
    lines = open(path).read().splitlines()
    # pandas writes an index column in front and True / False flags: both are read
    with open(path, "w") as fh:
        fh.write("\n".join(["," + lines[0]] + [f"{k},{line}" for k, line in enumerate(lines[1:])]) + "\n")
    assert np.array_equal(TrackTable.from_csv(path).bbox, table.bbox)
    broken = list(lines)
    broken[3] = broken[3].replace("[", "[[", 1)
    with open(path, "w") as fh:
        fh.write("\n".join(broken) + "\n")
    with pytest.raises(ValueError, match="line 4"):
        TrackTable.from_csv(path)
    with open(path, "w") as fh:
        fh.write("\n".join(line.split(",", 1)[1] for line in lines) + "\n")           # the track_id column cut off
    with pytest.raises(ValueError, match="track_id"):
        TrackTable.from_csv(path)


def test_track_rows_are_the_groups_in_file_order():
    table = big_table()
    for name, rows in table.track_rows.items():
        assert np.array_equal(rows, np.flatnonzero(table.track_id == name))
    assert sum(len(r) for r in table.track_rows.values()) == len(table)


# ------------------------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("ratio", [0, 0.1, 1])
def test_kept_negatives_follow_the_formula(ratio):
    table = big_table()
    n, neg = len(table), int((table.presence == 0).sum())
    want = max(0, int(min(neg / n, ratio) * n))
    assert kept_negatives(n, neg, ratio) == want
    s = TrackSampler(table, ratio, 10, 50, seed=1)
    assert int((table.presence[s.rows] == 0).sum()) == want and want == {0: 0, 0.1: 24, 1: neg}[ratio]
    assert int((table.presence[s.rows] == 1).sum()) == n - neg                 # every positive row stays
    assert np.all(np.diff(s.rows) > 0)
    other = TrackSampler(table, ratio, 10, 50, seed=2)
    if 0 < want < neg:
        assert not np.array_equal(other.rows, s.rows)                          # chosen at random
    for name, rows in s.track_rows.items():
        assert np.array_equal(rows, np.intersect1d(table.track_rows[name], s.rows))


def test_templates_are_present_and_not_near_corner():
    table = big_table()
    s = TrackSampler(table, 1, 10, 500, seed=0)
    assert s.num_tracks == 6 and len(s) == 500
    for _ in range(3):
        assert np.all(table.presence[s.epoch_rows] == 1) and not table.near_corner[s.epoch_rows].any()
        s.resample()
    want = np.flatnonzero((table.presence == 1) & ~table.near_corner)
    assert np.array_equal(s.template_rows, want)


def test_resample_gives_num_samples_in_both_branches():
    table = big_table()
    for n in (1, 6, 7, 100, 1000):                                           # with replacement: more samples than rows is fine
        s = TrackSampler(table, 0, 10, n, seed=n)
        assert len(s) == n == s.epoch_rows.size
        before = s.epoch_rows.copy()
        s.resample()
        assert len(s) == n and (n < 7 or not np.array_equal(before, s.epoch_rows))
    # per track ceil(n / tracks) draws with replacement, then a subset: no track can have more than that
    s = TrackSampler(table, 0, 10, 600, seed=9)
    counts = np.bincount(table.track_code[s.epoch_rows], minlength=6)
    assert counts.max() <= 100 and counts.sum() == 600
    # every template row its own track: without replacement
    n = 30
    single = TrackTable.from_arrays([f"t{k}" for k in range(n)], np.zeros(n), [f"{k}.jpg" for k in range(n)], np.ones((n, 4)), np.ones(n),
                                    np.zeros(n, bool), "d")
    s = TrackSampler(single, 0, 10, 20, seed=0)
    assert len(s) == 20 and np.unique(s.epoch_rows).size == 20
    s.resample()
    assert len(s) == 20 and np.unique(s.epoch_rows).size == 20
    assert TrackSampler(single, 0, 10, 30, seed=0).epoch_rows.size == 30
    with pytest.raises(ValueError):
        TrackSampler(single, 0, 10, 31, seed=0)


def test_resample_is_uniform_over_a_tracks_templates():
    table = big_table(tracks=2, per_track=12)
    s = TrackSampler(table, 0, 10, 20000, seed=4)
    for code in range(2):
        mine = s.template_rows[table.track_code[s.template_rows] == code]
        drawn = s.epoch_rows[table.track_code[s.epoch_rows] == code]
        assert drawn.size == 10000
        counts = np.array([(drawn == r).sum() for r in mine])
        p = 1 / mine.size
        assert np.all(np.abs(counts - drawn.size * p) < 4 * np.sqrt(drawn.size * p * (1 - p))), counts


@pytest.mark.parametrize("offset", [1, 4, 10, 31, 1000])
def test_clip_range_window_and_uniformity(offset):
    table = big_table()
    s = TrackSampler(table, 0.1, offset, 64, clip_range=True, seed=offset)
    got = s.pairs(np.arange(64))
    assert np.array_equal(got[:, 0], s.epoch_rows)
    assert np.array_equal(table.track_id[got[:, 0]], table.track_id[got[:, 1]])
    d = table.frame_index[got[:, 1]] - table.frame_index[got[:, 0]]
    assert np.all(np.abs(d) < offset) and np.isin(got[:, 1], s.rows).all()
    n = 20000
    for idx in (0, 17):
        template = s.epoch_rows[idx]
        track = s.track_rows[table.track_id[template]]
        candidates = track[np.abs(table.frame_index[track] - table.frame_index[template]) < offset]
        assert template in candidates
        drawn = s.pairs(np.full(n, idx))[:, 1]
        assert np.isin(drawn, candidates).all()
        counts = np.array([(drawn == r).sum() for r in candidates])
        p = 1 / candidates.size
        assert np.all(np.abs(counts - n * p) <= 4 * np.sqrt(n * p * (1 - p))), (offset, counts)
    if offset == 10:       # near_corner rows, kept negatives and both rows of a repeated frame are candidates somewhere
        drawn = s.pairs(np.tile(np.arange(64), 200))[:, 1]
        assert table.near_corner[drawn].any() and (table.presence[drawn] == 0).any()


def test_without_clip_range_the_search_row_is_uniform_over_the_track():
    table = big_table()
    s = TrackSampler(table, 1, 3, 16, clip_range=False, seed=2)
    n = 20000
    drawn = s.pairs(np.full(n, 5))[:, 1]
    track = s.track_rows[table.track_id[s.epoch_rows[5]]]
    assert track.size == 40
    counts = np.array([(drawn == r).sum() for r in track])
    p = 1 / track.size
    assert counts.sum() == n and np.all(np.abs(counts - n * p) < 4 * np.sqrt(n * p * (1 - p))), counts


def test_a_window_without_candidates_is_an_error():
    s = TrackSampler(big_table(), 0, 0, 8, clip_range=True, seed=0)
    with pytest.raises(ValueError):
        s.pair(0)
    with pytest.raises(IndexError):
        s.pairs([8])


@pytest.mark.parametrize("clip", [False, True])
def test_pairs_equals_pair_row_by_row(clip):
    table = big_table()
    a, b = (TrackSampler(table, 0.1, 7, 200, clip_range=clip, seed=11) for _ in range(2))
    indices = np.random.default_rng(0).integers(0, 200, 300)
    many = a.pairs(indices)
    one = np.stack([b.pair(int(i)) for i in indices])
    assert many.shape == (300, 2) and many.dtype == np.int64 and np.array_equal(many, one)
    assert np.array_equal(a.pairs(indices), np.stack([b.pair(int(i)) for i in indices]))      # and the streams stay together
    assert a.pairs([]).shape == (0, 2)


def test_pairs_does_no_work_of_the_tables_size(monkeypatch):
    """The bisection key of clip_range is made once per set of kept rows (`_index`), not per call: `pairs` touches B elements."""
    import feartracker_amd.train_data.sampling as sampling
    table = big_table()
    s = TrackSampler(table, 0.1, 7, 64, clip_range=True, seed=1)
    track, frame = table.track_code[s._by_track], table.frame_index[s._by_track]
    assert np.array_equal(s._key, track * s._span + (frame - s._base)) and np.all(np.diff(s._key) >= 0)
    assert s._span == frame.max() - frame.min() + 1 and s._key.size == s.rows.size
    key = s._key
    want = TrackSampler(table, 0.1, 7, 64, clip_range=True, seed=1).pairs(np.arange(64))

    class Sized(np.ndarray):                     # an array that refuses whole-array passes
        def _no(self, *a, **k):
            raise AssertionError("pairs() made a pass over a table-sized array")
        min = max = sum = argsort = __mul__ = __add__ = __sub__ = _no
    s._key, s._frame = s._key.view(Sized), s._frame.view(Sized)
    monkeypatch.setattr(sampling.np, "repeat", Sized._no)
    assert np.array_equal(s.pairs(np.arange(64)), want)
    monkeypatch.undo()
    assert s._key.base is key or s._key is key
    s.resample()
    s.frame_offset = 3                          # neither resampling nor another offset needs a new key
    assert np.all(np.abs(table.frame_index[s.pairs(np.arange(64))] @ [1, -1]) < 3)
    state = s.state_dict()
    state["rows"] = state["rows"][:-3]
    s.load_state_dict(state)                    # other kept rows: a new key
    assert s._key.size == s.rows.size == key.size - 3


def test_update_offset_on_the_shipped_got10k_values():
    cfg = dict(start_epoch=20, freq=5, step=5, max_value=150)
    offset, seen = 70, {}
    for epoch in range(120):
        new = update_offset(offset, epoch, **cfg)
        if new != offset:
            seen[epoch] = (offset, new)
        offset = new
    assert min(seen) == 19 and seen[19] == (70, 75) and seen[24] == (75, 80) and 20 not in seen and 14 not in seen
    assert offset == 150 and max(seen) == 94 and seen[94] == (145, 150)
    # through the plan, on every sampler
    table = big_table()
    samplers = [TrackSampler(table, 0, 70, 40, clip_range=True, seed=k) for k in range(2)]
    plan = EpochPlan(samplers, 8, seed=0)
    for epoch in range(20):
        rows = [s.epoch_rows.copy() for s in samplers]
        plan.end_epoch(epoch, cfg)
        assert all(not np.array_equal(r, s.epoch_rows) for r, s in zip(rows, samplers))       # resampled
        assert all(s.frame_offset == (75 if epoch >= 19 else 70) for s in samplers)
    plan.end_epoch(20, None)
    assert all(s.frame_offset == 75 for s in samplers)


# ---------------------------------------------------------------------------------------------------------------------------- plan
def test_epoch_plan_one_rank():
    table = big_table()
    samplers = [TrackSampler(table, 0, 5, 37, seed=0), TrackSampler(table, 0, 5, 30, seed=1)]
    plan = EpochPlan(samplers, 8, seed=3)
    assert len(plan) == 67 // 8
    first = plan.start_epoch()
    assert first.shape == (8, 8) and np.unique(first).size == 64 and first.min() >= 0 and first.max() < 67
    second = plan.start_epoch()
    assert second.shape == (8, 8) and not np.array_equal(first, second)
    which, index = plan.locate(np.arange(67))
    assert np.array_equal(which, np.repeat([0, 1], [37, 30])) and np.array_equal(index, np.concatenate([np.arange(37), np.arange(30)]))
    whole = EpochPlan(samplers, 1, seed=3).start_epoch()
    assert np.array_equal(np.sort(whole.reshape(-1)), np.arange(67))            # a permutation of the epoch
    assert np.array_equal(whole.reshape(-1)[:64], first.reshape(-1))            # cut into full batches, the rest dropped


def test_epoch_plan_two_ranks():
    table = big_table()
    sampler = TrackSampler(table, 0, 5, 67, seed=0)
    plans = [EpochPlan([sampler], 1, seed=3, rank=r, world=2) for r in range(2)]
    parts = [p.start_epoch().reshape(-1) for p in plans]
    assert parts[0].size == parts[1].size == 34
    whole = EpochPlan([sampler], 1, seed=3).start_epoch().reshape(-1)
    assert np.array_equal(parts[0], np.concatenate([whole, whole[:1]])[0::2])
    assert np.array_equal(parts[1], np.concatenate([whole, whole[:1]])[1::2])
    both = np.concatenate(parts)
    assert np.array_equal(np.unique(both), np.arange(67))                       # together they cover the epoch
    values, counts = np.unique(both, return_counts=True)
    assert counts.sum() == 68 and values[counts == 2].tolist() == [int(whole[0])]    # disjoint but for the wrapped tail
    batched = [EpochPlan([sampler], 8, seed=3, rank=r, world=2) for r in range(2)]
    assert all(len(p) == 4 and p.start_epoch().shape == (4, 8) for p in batched)
    with pytest.raises(ValueError):
        EpochPlan([sampler], 8, seed=0, rank=2, world=2)


def test_states_continue_draw_for_draw():
    table = big_table()

    def make():
        samplers = [TrackSampler(table, 0.1, 6, 50, clip_range=True, seed=k) for k in range(2)]
        return samplers, EpochPlan(samplers, 8, seed=5)
    samplers, plan = make()
    plan.start_epoch()
    samplers[0].pairs(np.arange(10))
    plan.end_epoch(0, dict(start_epoch=1, freq=1, step=3, max_value=100))
    state = plan.state_dict()
    others, restored = make()
    others[0].rows = others[0].rows[:-1]                                        # (the kept rows come from the state too)
    restored.load_state_dict(state)
    assert [s.frame_offset for s in others] == [9, 9]
    for _ in range(2):
        assert np.array_equal(plan.start_epoch(), restored.start_epoch())
        for s, o in zip(samplers, others):
            assert np.array_equal(s.epoch_rows, o.epoch_rows) and np.array_equal(s.rows, o.rows)
            assert np.array_equal(s.pairs(np.arange(50)), o.pairs(np.arange(50)))
        plan.end_epoch(1, None)
        restored.end_epoch(1, None)
    single = TrackSampler(table, 0.1, 6, 50, seed=8)
    saved = single.state_dict()
    want = (single.pairs(np.arange(50)), single.resample(), single.epoch_rows.copy())
    single.load_state_dict(saved)
    assert np.array_equal(single.pairs(np.arange(50)), want[0])
    single.resample()
    assert np.array_equal(single.epoch_rows, want[2])


# ------------------------------------------------------------------------------------------------------------------------ clipping
def test_clip_boxes_equals_ensure_bbox_boundaries():
    shapes = [(64, 96), (72, 80)]
    boxes = [[-5, 10, 20, 20], [10, -5.5, 20, 20], [90, 10, 20.7, 20], [10, 60, 20, 20], [-10, -10, 200, 200], [200, 200, 5, 5],
             [-30, -30, 10, 10], [3.9, 4.2, 10.6, 7.5], [0, 0, 96, 64], [95.5, 63.5, 3, 3], [10, 10, 0, 0], [10, 10, -4, 5]]
    rng = np.random.default_rng(0)
    boxes += rng.uniform(-40, 130, size=(200, 4)).tolist()
    for shape in shapes:
        want = np.stack([ensure_bbox_boundaries(b, shape) for b in boxes])
        got = clip_boxes(np.array(boxes), np.tile(shape, (len(boxes), 1)))
        assert got.dtype == np.int32 and np.array_equal(got, want)
    mixed = clip_boxes(np.array(boxes[:4]), np.array([shapes[k % 2] for k in range(4)]))
    assert np.array_equal(mixed, np.stack([ensure_bbox_boundaries(b, shapes[k % 2]) for k, b in enumerate(boxes[:4])]))
