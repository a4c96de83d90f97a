"""bench.py's contract: a plain run times exactly --steps steps and prints the headline line without the --full extras, and
--dump-outputs writes what the last timed step computed (losses, a fixed sample of the parameters and gradients, the module
buffers) as float32 / float64 .npy files within 64 MB, the same bit for bit on every run with the same arguments."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_trainer(n, seed):
    g = torch.Generator().manual_seed(seed)
    flat_p, flat_g = torch.randn(n + 64, generator=g), torch.randn(n + 64, generator=g)
    net = torch.nn.BatchNorm2d(3)
    opt = types.SimpleNamespace(flat_p=flat_p, flat_g=flat_g, gather=lambda f: torch.cat([f[:n // 2], f[n // 2 + 64:n + 64]]))
    return types.SimpleNamespace(opt=opt, nets=[net, None])


def test_output_snapshot_is_a_fixed_sample(monkeypatch, tmp_path):
    assert 2 * 4 * bench.DUMP_SAMPLE <= 48 << 20          # the full-size bucket: two sampled float32 vectors + small buffers
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    losses = {"loss": torch.tensor(1.5), "loss_2": 0}
    a = bench.output_snapshot(_fake_trainer(5000, 0), losses)
    b = bench.output_snapshot(_fake_trainer(5000, 1), losses)
    assert a["loss"].dtype == np.float64 and float(a["loss"]) == 1.5 and float(a["loss_2"]) == 0.0
    assert a["params"].dtype == np.float32 and a["grads"].dtype == np.float32 and a["buffers"].dtype == np.float64
    assert 900 < a["params"].size <= 1000 and a["params"].shape == a["grads"].shape == b["params"].shape
    # the sample positions: recovered from buckets that hold their own indices -- sorted, the same for the parameters and the
    # gradients, and the same on every call whatever the values
    pos = []
    for seed in (0, 1):
        tr = _fake_trainer(5000, seed)
        tr.opt.flat_p = torch.arange(5064, dtype=torch.float32)
        tr.opt.flat_g = torch.arange(5064, dtype=torch.float32)
        s_ = bench.output_snapshot(tr, losses)
        np.testing.assert_array_equal(s_["params"], s_["grads"])
        pos.append(s_["params"])
    np.testing.assert_array_equal(pos[0], pos[1])
    assert np.all(np.diff(pos[0]) > 0) and 900 < pos[0].size <= 1000
    # ... and the values at those positions
    flat_p = _fake_trainer(5000, 0).opt.flat_p
    np.testing.assert_array_equal(a["params"], flat_p.numpy()[pos[0].astype(np.int64)])
    small = bench.output_snapshot(_fake_trainer(800, 0), losses)            # below the sample size: every element
    assert small["params"].size == 800
    bench.dump_outputs(str(tmp_path / "out"), a)
    for k, v in a.items():
        np.testing.assert_array_equal(np.load(str(tmp_path / "out" / (k + ".npy"))), v)


def _plain_run(out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
           "--height", "128", "--width", "192", "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    out = str(tmp_path / "dump")
    line = _plain_run(out)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "images/s" and line["dtype"] == "f32"
    assert abs(line["value"] - 2e3 / line["ms_per_step"]) <= 1e-2 * line["value"]        # 2 images per step
    assert "cpu_baseline" not in line and "parity" not in line and line["roofline"] is None and line["kernels"] is None
    files = sorted(os.listdir(out))
    assert {"loss.npy", "params.npy", "grads.npy", "buffers.npy"} <= set(files)
    total = 0
    for f in files:
        v = np.load(os.path.join(out, f))
        assert v.dtype in (np.float32, np.float64) and np.all(np.isfinite(v)), f
        total += os.path.getsize(os.path.join(out, f))
    assert total <= 64 << 20
    assert abs(float(np.load(os.path.join(out, "loss.npy"))) - line["config"]["loss"]) <= 1e-5 * abs(line["config"]["loss"]) + 1e-6
    # the same arguments: the same outputs, bit for bit
    out2 = str(tmp_path / "dump2")
    _plain_run(out2)
    assert sorted(os.listdir(out2)) == files
    for f in files:
        assert np.array_equal(np.load(os.path.join(out, f)), np.load(os.path.join(out2, f))), f
