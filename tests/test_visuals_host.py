"""The numpy statements of the drawing operator and the best / worst miner (feartracker_amd/visuals.py), the struct mirror, and the
operators' statuses that need no GPU.  `draw_boxes_host` is pinned to the rectangle contract by a brute-force per-pixel predicate written
from include/fear_train.h's statement, not from the slicing code."""
import ctypes
import subprocess

import numpy as np
import pytest

import metricsgen as mg
import visualsgen as vg
from feartracker_amd import train_abi, visuals as V
from feartracker_amd.metrics import step_metrics_host

ROOT = vg.__file__.rsplit("/tests/", 1)[0]


def _band(h, w, box, t):
    """The contract, pixel by pixel: in the outer rectangle and not in the inner one."""
    x, y, bw, bh = (int(v) for v in box)
    x0, x1, y0, y1 = min(x, x + bw), max(x, x + bw), min(y, y + bh), max(y, y + bh)
    o, i = t // 2, (t - 1) // 2
    py, px = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]      # every pixel, evaluated on its own
    outer = (x0 - o <= px) & (px <= x1 + o) & (y0 - o <= py) & (py <= y1 + o)
    inner = (x0 + i + 1 <= px) & (px <= x1 - i - 1) & (y0 + i + 1 <= py) & (py <= y1 - i - 1)
    return outer & ~inner


def _brute(frames, boxes, frame_of, colours, t):
    out = [f.copy() for f in frames]
    for k, box in enumerate(boxes):
        f = int(frame_of[k])
        if 0 <= f < len(out):
            out[f][_band(out[f].shape[0], out[f].shape[1], box, t)] = colours[k]
    return out


@pytest.mark.parametrize("t", (1, 2, 3, 5, 32))
@pytest.mark.parametrize("shape", ((1, 1), (4, 4), (37, 70)))
def test_band_rule_equals_the_per_pixel_predicate(shape, t):
    h, w = shape
    for k, box in enumerate(vg.edge_boxes(h, w)):
        img = vg.frame(h, w, k)
        want = img.copy()
        mask = _band(h, w, box, t)
        want[mask] = (1, 2, 3)
        V.draw_boxes_host([img], [box], [0], (1, 2, 3), t)
        np.testing.assert_array_equal(img, want, err_msg=f"box {box.tolist()} t={t}")


def test_band_width_and_the_named_cases():
    img = np.zeros((40, 40, 3), np.uint8)
    for t in (1, 2, 5):
        img[:] = 0
        V.draw_boxes_host([img], [(10, 10, 15, 12)], [0], (255, 255, 255), t)
        row = np.flatnonzero(img[16, :, 0])                 # a row through the middle: two runs of exactly t pixels
        o = t // 2
        assert row.tolist() == list(range(10 - o, 10 - o + t)) + list(range(25 - (t - 1) // 2, 25 - (t - 1) // 2 + t))
        assert img[10 - o, 10 - o, 0] == 255                # square corners
    img[:] = 0
    V.draw_boxes_host([img], [(60, 60, 5, 5), (-30, 2, 4, 4)], [0, 0], (9, 9, 9), 5)
    assert not img.any()                                    # wholly outside
    V.draw_boxes_host([img], [(5, 5, 2, 30)], [0], (9, 9, 9), 5)
    assert (img[3:38, 3:10] == 9).all() and img.sum() == 9 * 3 * 35 * 7          # thinner than the band: filled
    with pytest.raises(ValueError):
        V.draw_boxes_host([img], [(1, 1, 2, 2)], [0], (9, 9, 9), 33)


@pytest.mark.parametrize("n", (2, 3))
def test_swapping_the_order_changes_exactly_the_intersection(n):
    h, w, t = 48, 64, 5
    boxes = np.array([(8, 6, 30, 24), (20, 14, 30, 24), (14, 2, 12, 40)], dtype=np.int32)[:n]
    cols = np.array([(200, 0, 0), (0, 200, 0), (0, 0, 200)], dtype=np.uint8)[:n]
    base = vg.frame(h, w, 1)
    fwd = V.draw_boxes_host([base.copy()], boxes, None, cols, t)[0]
    rev = V.draw_boxes_host([base.copy()], boxes[::-1], None, cols[::-1], t)[0]
    bands = np.stack([_band(h, w, b, t) for b in boxes])
    shared = bands.sum(axis=0) >= 2
    assert shared.any()
    differ = (fwd != rev).any(axis=2)
    np.testing.assert_array_equal(differ, shared)           # (the colours differ, so every shared pixel changes)
    last = np.array([np.flatnonzero(bands[:, y, x]).max() if bands[:, y, x].any() else -1 for y in range(h) for x in range(w)]).reshape(h, w)
    for k in range(n):
        assert (fwd[last == k] == cols[k]).all()
    np.testing.assert_array_equal(fwd[last < 0], base[last < 0])


def test_every_operator_case_equals_the_per_pixel_predicate():
    for name, shapes, boxes, frame_of, cols, t in vg.draw_cases():
        frames = [vg.frame(h, w, i) for i, (h, w) in enumerate(shapes)]
        want = _brute(frames, boxes, frame_of, cols, t)
        got = V.draw_boxes_host([f.copy() for f in frames], boxes, frame_of, cols, t)
        for g, wnt in zip(got, want):
            np.testing.assert_array_equal(g, wnt, err_msg=name)


def test_two_frames_and_indices_out_of_range():
    a, b = vg.frame(20, 30, 1), vg.frame(9, 50, 2)
    boxes = [(2, 2, 10, 10), (30, 1, 12, 5), (1, 1, 3, 3), (1, 1, 3, 3)]
    got = V.draw_boxes_host([a.copy(), b.copy()], boxes, [0, 1, -1, 2], [(1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4)], 1)
    assert (got[0][2, 2:13] == 1).all() and (got[1][1, 30:43] == 2).all()
    assert not (got[0] == 3).all(axis=2).any() and not (got[1] == 4).all(axis=2).any()
    assert (got[0] != a).any(axis=2).sum() == 40 and (got[1] != b).any(axis=2).sum() <= 2 * 13 + 2 * 4
    only = V.draw_boxes_host([a.copy()], [(1, 1, 3, 3)], [5], (3, 3, 3), 5)[0]
    np.testing.assert_array_equal(only, a)


# ---------------------------------------------------------------------------------------------------------------- the miner
def _decisions(scores, mode, min_delta):
    state, out = V.miner_state_host(), []
    for step, s in enumerate(scores):
        out.append(V.miner_decide_host(state, s, mode == "max", min_delta, step))
    return out, state


def test_decision_sequences():
    nan = float("nan")
    # mode min: first step | a tie within min_delta | better | worse | equal to best - min_delta exactly
    took, st = _decisions([1.0, 1.05, 0.5, 2.0, 0.4, 0.45], "min", 0.1)
    assert took == [(1, 1), (0, 0), (1, 0), (0, 1), (1, 0), (0, 0)]
    assert st["score"].tolist() == [0.4, 2.0] and st["step"].tolist() == [4, 3] and st["has"].tolist() == [1, 1]
    took, st = _decisions([1.0, 1.05, 0.5, 2.0], "max", 0.1)
    assert took == [(1, 1), (0, 0), (0, 1), (1, 0)] and st["score"].tolist() == [2.0, 0.5]
    # the boundary is inclusive, as the reference's <= and >=
    assert _decisions([1.0, 0.75, 1.25], "min", 0.25)[0] == [(1, 1), (1, 0), (0, 1)]
    # a NaN first stays on both sides; a NaN later takes nothing
    took, st = _decisions([nan, 0.1, 5.0], "min", 1e-4)
    assert took == [(1, 1), (0, 0), (0, 0)] and np.isnan(st["score"]).all() and st["step"].tolist() == [0, 0]
    took, st = _decisions([1.0, nan, 0.5], "max", 1e-4)
    assert took == [(1, 1), (0, 0), (0, 1)] and st["score"].tolist() == [1.0, 0.5]


def test_denormalisation_of_every_level_stays_within_one_below():
    from feartracker_amd.train_data import _normalise_u8
    levels = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)           # (256, 1, 3): every level in every channel
    back = V.denormalise_host(_normalise_u8(levels)).astype(np.int64)
    d = levels.astype(np.int64) - back
    print("levels that come back one below:", int((d == 1).sum()), "of", d.size)
    assert d.min() >= 0 and d.max() <= 1
    odd = np.array([np.nan, np.inf, -np.inf, 9.0, -9.0, 0.0], dtype=np.float32).reshape(1, 1, 6).repeat(3, axis=0)
    assert V.denormalise_host(odd)[0, :5].tolist() == [[0] * 3, [255] * 3, [0] * 3, [255] * 3, [0] * 3]


def test_truncation_of_decoded_boxes():
    b = np.array([[1.9, -1.9, 0.5, -0.5], [np.nan, np.inf, -np.inf, 3e9], [2.0 ** 20 + 0.5, -(2.0 ** 20) - 7, 255.99, -0.0]])
    assert V.truncate_boxes_host(b).tolist() == [[1, -1, 0, 0], [0, 1 << 20, -(1 << 20), 1 << 20], [1 << 20, -(1 << 20), 255, 0]]


@pytest.mark.parametrize("B,n_images", ((3, 2), (2, 16)))
def test_miner_host_layout_colours_and_boxes(B, n_images):
    m = vg.miner_step(B, 1)
    n = min(B, n_images)
    state, sheets = V.miner_host(V.miner_state_host(), None, m["template"], m["search"], m["cls"], m["bbox"], m["gt_box"], m["visible"],
                                 (0.25, 0.5), n_images, "min", 1e-4, step=7)
    assert sheets.shape == (2, n * 256, 384, 3) and state["take"].tolist() == [1, 1] and state["step"].tolist() == [7, 7]
    assert state["score"].tolist() == [0.75, 0.75]
    np.testing.assert_array_equal(sheets[0], sheets[1])
    with np.errstate(invalid="ignore"):                                            # (the planted non-finite cell)
        host = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], m["visible"], m["dataset_id"], mg.N_DATASETS)
        want = V.truncate_boxes_host(host["boxes"][:n])
    np.testing.assert_array_equal(state["pred"][:n], want)
    assert (state["pred"][n:] == 0).all()
    assert m["visible"][0] != 0 and m["visible"][1] == 0 and n >= 2                # both colours are rendered
    for k in range(n):
        item = sheets[0][256 * k:256 * (k + 1)]
        np.testing.assert_array_equal(item[:128, :128], V.denormalise_host(m["template"][k]))
        assert not item[128:, :128].any()                                       # hstack_autopad's padding
        crop = V.denormalise_host(m["search"][k])
        gt_band = _band(256, 256, m["gt_box"][k], 2)
        pred_band = _band(256, 256, want[k], 2) & ~gt_band
        assert gt_band.any()
        assert (item[:, 128:][gt_band] == ((250, 0, 0) if m["visible"][k] else (0, 0, 250))).all()
        assert (item[:, 128:][pred_band] == (0, 250, 0)).all()
        rest = ~(gt_band | pred_band)
        np.testing.assert_array_equal(item[:, 128:][rest], crop[rest])
    # a step that neither side takes leaves state and sheets alone but for take
    m2 = vg.miner_step(B, 2)
    state2, sheets2 = V.miner_host(state, sheets, m2["template"], m2["search"], m2["cls"], m2["bbox"], m2["gt_box"], m2["visible"],
                                   (0.75,), n_images, "min", 1e-4, step=8)
    assert state2["take"].tolist() == [0, 0] and state2["step"].tolist() == [7, 7]
    np.testing.assert_array_equal(sheets2, sheets)
    np.testing.assert_array_equal(state2["pred"], state["pred"])
    # worst only: the other sheet keeps the first batch
    state3, sheets3 = V.miner_host(state2, sheets2, m2["template"], m2["search"], m2["cls"], m2["bbox"], m2["gt_box"], m2["visible"],
                                   (1.0, 1.0), n_images, "min", 1e-4, step=9)
    assert state3["take"].tolist() == [0, 1] and state3["step"].tolist() == [7, 9] and state3["score"].tolist() == [0.75, 2.0]
    np.testing.assert_array_equal(sheets3[0], sheets[0])
    assert (sheets3[1] != sheets[1]).any()


def test_the_score_is_added_in_fp32():
    m = vg.miner_step(2, 0)
    a, b = np.float32(0.1), np.float32(1e-9)
    state, _ = V.miner_host(V.miner_state_host(), None, m["template"], m["search"], m["cls"], m["bbox"], m["gt_box"], m["visible"], (a, b), 1)
    assert state["score"][0] == float(np.float32(a + b)) == float(a)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_miner_state_mirror_has_the_headers_layout(tmp_path):
    cls = train_abi.FearMinerState
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fear_train.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(FearMinerState));']
    lines += [f'  printf("{field} %zu\\n", offsetof(FearMinerState, {field}));' for field, _ in cls._fields_]
    lines += ['  printf("max %d\\n", FEAR_MINER_MAX_IMAGES);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("size")) == ctypes.sizeof(cls) == V.MINER_STATE_DTYPE.itemsize == 1072
    assert int(out.pop("max")) == train_abi.FEAR_MINER_MAX_IMAGES == 64
    assert {k: int(v) for k, v in out.items()} == {field: getattr(cls, field).offset for field, _ in cls._fields_}
    assert [V.MINER_STATE_DTYPE.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]


def test_symbols_and_statuses_that_need_no_gpu():
    assert {"fear_draw_boxes_u8", "fear_miner_update"} <= set(train_abi.TRAIN_SYMBOLS)
    import feartracker_amd
    for name in ("BestWorstMiner", "draw_boxes", "draw_boxes_host", "miner_host"):
        assert name in feartracker_amd.__all__ and hasattr(feartracker_amd, name)
    assert hasattr(feartracker_amd.FEARMultiTracker, "draw")
    lib = train_abi.load_train_library()
    OK, NULL, SHAPE = 0, -1, -2
    fake = ctypes.c_void_p(4096)
    draw = lib.fear_draw_boxes_u8
    assert draw(None, 3, None, None, None, 0, 5, None) == OK and draw(None, 0, None, None, None, 4, 5, None) == OK
    assert draw(None, 1, fake, fake, fake, 1, 5, None) == NULL and draw(fake, 1, None, fake, fake, 1, 5, None) == NULL
    assert draw(fake, 1, fake, None, fake, 1, 5, None) == NULL and draw(fake, 1, fake, fake, None, 1, 5, None) == NULL
    assert draw(fake, 1, fake, fake, fake, 65536, 5, None) == SHAPE and draw(fake, -1, fake, fake, fake, 1, 5, None) == SHAPE
    assert draw(fake, 1, fake, fake, fake, 1, 0, None) == SHAPE and draw(fake, 1, fake, fake, fake, 1, 33, None) == SHAPE
    assert draw(fake, 1, fake, fake, fake, -1, 5, None) == SHAPE
    miner = lib.fear_miner_update
    args = [fake] * 8
    assert miner(*([None] * 8), 0, 16, 0, 1e-4, 0, None, None, None) == OK
    assert miner(*args, 4, 0, 0, 1e-4, 0, fake, fake, None) == SHAPE and miner(*args, 4, 65, 0, 1e-4, 0, fake, fake, None) == SHAPE
    assert miner(*args, 65536, 16, 0, 1e-4, 0, fake, fake, None) == SHAPE and miner(*args, -1, 16, 0, 1e-4, 0, fake, fake, None) == SHAPE
    for missing in (0, 1, 2, 3, 4, 5, 6):
        a = list(args)
        a[missing] = None
        assert miner(*a, 4, 16, 0, 1e-4, 0, fake, fake, None) == NULL
    assert miner(*args, 4, 16, 0, 1e-4, 0, None, fake, None) == NULL and miner(*args, 4, 16, 0, 1e-4, 0, fake, None, None) == NULL


def test_host_arguments_are_checked_without_a_gpu():
    with pytest.raises(ValueError):
        V.BestWorstMiner("cpu", max_images=0)
    with pytest.raises(ValueError):
        V.BestWorstMiner("cpu", max_images=65)
    with pytest.raises(ValueError):
        V.BestWorstMiner("cpu", metric_mode="median")
    assert V.BestWorstMiner("cpu").sheets() == {}
    import torch
    with pytest.raises(ValueError):
        V.draw_boxes(torch.zeros(4, 4, 3, dtype=torch.uint8), [(0, 0, 1, 1)])                  # a host frame
    with pytest.raises(ValueError):
        V.draw_boxes([], [(0, 0, 1, 1)])
