"""bench.py's command line: a plain run prints the headline line only, `--dump-outputs DIR`
writes what the timed path left behind (the same arrays from run to run), `--full` adds the
other legs.  The sampling of dump_outputs is checked on the CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_when_small(tmp_path):
    import torch

    import bench
    arrs = {"a": torch.arange(12.0).view(3, 4), "n": torch.tensor(7), "d": np.arange(5.0)}
    bench.dump_outputs(str(tmp_path / "o"), arrs)
    a = np.load(tmp_path / "o" / "a.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4)
    np.testing.assert_array_equal(a, np.arange(12.0).reshape(3, 4))
    n = np.load(tmp_path / "o" / "n.npy")
    assert n.dtype == np.float64 and n == 7
    assert np.load(tmp_path / "o" / "d.npy").dtype == np.float64


def test_dump_outputs_samples_above_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    rs = np.random.RandomState(3)
    arrs = {"small": rs.randn(100).astype(np.float32),          # 400 B: below the share, whole
            "big": rs.randn(50, 40).astype(np.float32),          # 8000 B
            "big2": rs.randn(2000).astype(np.float32),           # same size: same positions
            "wide": rs.randn(3000)}                              # float64, 24000 B
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), arrs)
    got = {k: np.load(tmp_path / "x" / (k + ".npy")) for k in arrs}
    assert sum(v.nbytes for v in got.values()) <= 4000
    np.testing.assert_array_equal(got["small"], arrs["small"])
    share = (4000 - 400) // 3
    assert got["big"].shape == (share // 4,) and got["wide"].shape == (share // 8,)
    # a sample of the array's own elements, in their order, at the same positions for equal sizes
    flat = arrs["big"].reshape(-1)
    pos = np.flatnonzero(np.isin(flat, got["big"]))
    np.testing.assert_array_equal(flat[pos], got["big"])
    np.testing.assert_array_equal(arrs["big2"][pos], got["big2"])
    assert pos.max() > flat.size * 0.9 and pos.min() < flat.size * 0.1
    for k in arrs:                                               # the same elements every time
        np.testing.assert_array_equal(got[k], np.load(tmp_path / "y" / (k + ".npy")))


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "16",
                        "--warmup", "4"] + list(extra), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_reproducible_dump(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res = _bench("--dump-outputs", a)
    assert res["metric"] == "acoustic frames/sec (train)" and res["unit"] == "frames/s"
    assert res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["steps"] == 16 and res["warmup"] == 4 and res["ms_per_step"] > 0
    # value is frames over the timed steps: 16 batches of 128 frames at ms_per_step each
    assert res["value"] == pytest.approx(128 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    # the other legs stay behind --full
    for k in ("roofline", "step_breakdown_us", "cpu_baseline", "fp32_entry", "sequence_configs",
              "batch_sweep_frames_per_s", "posterior_max_rel_err"):
        assert k not in res
    _bench("--dump-outputs", b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    for want in ("loss_err.npy", "chunk_totals.npy", "out_dnn2.npy", "out_dnn3.npy",
                 "MLP_layers1.wx.0.weight.npy", "MLP_layers2.wx.0.weight.npy"):
        assert want in names
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 * 1000 * 1000
    post = np.load(os.path.join(a, "out_dnn2.npy"))
    assert post.shape == (128, 1928)
    np.testing.assert_allclose(np.exp(post.astype(np.float64)).sum(1), 1.0, atol=1e-3)
    # 3 untimed eager steps + warm-up + the timed steps, every one of them run
    assert np.load(os.path.join(a, "MLP_layers1.bn.0.num_batches_tracked.npy")) == 3 + 4 + 16
