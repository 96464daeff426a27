"""The driver's contract with bench.py: ONE JSON line on stdout with the keys the prompt names, `roofline` and `cpu_baseline`
objects under --full, N=1 defaults; a plain run carries the headline keys only and --dump-outputs writes the last timed step's
maps; `--gpus 2` on a box without two GPUs fails with a message about GPUs, not about the launcher."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_without_the_gpus_fails_cleanly():
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs present")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode != 0
    assert "GPU" in (res.stderr + res.stdout) and "torch.distributed.run" not in res.stderr.splitlines()[-1]


@pytest.mark.gpu
def test_one_json_line_with_the_contract_keys():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "3", "--full", "--no-fear-m", "--no-train",
                          "--no-latency", "--no-pipelined"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                                   # exactly one line on stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 3 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and "workload" in d["config"]
    assert abs(d["value"] - 256 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.0 < r["frac"] < 1.0 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]


HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config")
FULL_ONLY_KEYS = ("roofline", "cpu_baseline", "other_math_mode", "device_under_load", "pipelined_two_streams", "split_streams_option",
                  "config5_train_step", "config4_fear_m_bf16", "latency_batch1")


def test_dump_outputs_writes_float_arrays_and_samples_past_the_limit(tmp_path):
    """bench.dump_outputs: one .npy per name, dtype kept; beyond the byte limit the same seeded, ordered sample of crops of every
    array, the same sample on every call."""
    import numpy as np
    import bench
    rng = np.random.RandomState(1)
    bbox = rng.rand(40, 4, 16, 16).astype(np.float32)
    cls = rng.rand(40, 1, 16, 16).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "all"), {"bbox": bbox, "cls": cls})
    assert np.array_equal(np.load(tmp_path / "all" / "bbox.npy"), bbox) and np.load(tmp_path / "all" / "cls.npy").dtype == np.float32
    limit = (bbox.nbytes + cls.nbytes) // 4
    for sub in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / sub), {"bbox": bbox, "cls": cls}, limit=limit)
    b1, c1 = np.load(tmp_path / "s1" / "bbox.npy"), np.load(tmp_path / "s1" / "cls.npy")
    assert b1.nbytes + c1.nbytes <= limit and b1.shape[0] == c1.shape[0] == 10
    assert np.array_equal(b1, np.load(tmp_path / "s2" / "bbox.npy"))
    rows = [int(np.flatnonzero((bbox == r).all(axis=(1, 2, 3)))[0]) for r in b1]
    assert rows == sorted(rows) and all(np.array_equal(cls[i], c) for i, c in zip(rows, c1))
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "bad"), {"ids": np.arange(4)})


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run prints the headline keys only (nothing that --full adds), and --dump-outputs holds the maps the engine computes
    for the bench's seeded inputs."""
    import numpy as np
    import torch
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--batch", "16",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in HEADLINE_KEYS:
        assert k in d, k
    assert not [k for k in FULL_ONLY_KEYS if k in d]
    assert d["steps"] == 4 and d["warmup"] == 2 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    bbox, cls = np.load(tmp_path / "bbox.npy"), np.load(tmp_path / "cls.npy")
    assert bbox.shape == (16, 4, 16, 16) and cls.shape == (16, 1, 16, 16) and bbox.dtype == cls.dtype == np.float32
    sys.path.insert(0, ROOT)
    import bench
    from feartracker_amd import DEFAULT_WEIGHTS, FEARNetHIP
    search_u8, tmpl_u8 = bench.synth_batch(16, 0)
    net = FEARNetHIP(DEFAULT_WEIGHTS, device=0, max_batch=256)
    z = net.get_features(bench.norm_u8(tmpl_u8.cuda()).contiguous())
    rb, rc = net.track_maps(bench.norm_u8(search_u8.cuda()).contiguous(), z)
    torch.cuda.synchronize()
    np.testing.assert_allclose(bbox, rb.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(cls, rc.cpu().numpy(), rtol=1e-5, atol=1e-5)
