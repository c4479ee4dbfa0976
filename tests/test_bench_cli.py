"""bench.py's command line: a plain run measures the headline path only and can dump what its last timed step left;
everything else sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_plain_run_switches_every_leg_off(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert all(getattr(a, "no_" + leg) for leg in bench.LEGS)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-sweep"])
    a = bench.parse()
    assert a.full and a.no_sweep
    assert not any(getattr(a, "no_" + leg) for leg in bench.LEGS if leg != "sweep")


def test_write_outputs_float32_and_size_cap(tmp_path, monkeypatch):
    bench = _bench()
    small = torch.arange(10, dtype=torch.float64)
    bench.write_outputs(str(tmp_path / "a"), {"loss": small[:1], "params": small})
    x = np.load(tmp_path / "a" / "params.npy")
    assert x.dtype == np.float32 and np.array_equal(x, np.arange(10, dtype=np.float32))
    assert sorted(os.listdir(tmp_path / "a")) == ["loss.npy", "params.npy"]
    # an array over its share of the budget: a fixed sample, the same in every run, with its indices
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096)
    big = torch.arange(5000, dtype=torch.float32) * 0.5
    for d in ("b", "c"):
        bench.write_outputs(str(tmp_path / d), {"loss": small[:1], "params": big})
    xb, ib = np.load(tmp_path / "b" / "params.npy"), np.load(tmp_path / "b" / "params_index.npy")
    assert np.array_equal(xb, np.load(tmp_path / "c" / "params.npy"))
    assert np.array_equal(ib, np.load(tmp_path / "c" / "params_index.npy"))
    assert xb.dtype == np.float32 and ib.dtype == np.float64 and 0 < xb.size == ib.size < 5000
    assert np.array_equal(xb, ib.astype(np.float32) * 0.5) and np.all(np.diff(ib) > 0)
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 4096


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run on a small scene: the line has the headline keys and no --full record, --steps sets the timed
    steps, and the dump holds the loss, parameters and gradients of the last timed step as finite float32."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--train-views", "2", "--batch", "512", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "rays/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    # value is rays per second of the timed steps: batch / step time (ms_per_step is rounded to 3 decimals)
    assert out["value"] == pytest.approx(512 / (out["ms_per_step"] * 1e-3), rel=0.0006 / out["ms_per_step"] + 1e-4)
    assert out["roofline"] is None and out["cpu_baseline"] is None
    for k in ("dropin", "bf16", "psnr", "llff", "sweep", "ngp", "container", "fp32_native_gemm"):
        assert k not in out, k
    from nerf_amd.vanilla import PackedLayout
    n = 2 * PackedLayout.get().total
    loss, params, grads = (np.load(out_dir / f"{k}.npy") for k in ("loss", "params", "grads"))
    assert loss.dtype == params.dtype == grads.dtype == np.float32
    assert loss.shape == (1,) and params.shape == (n,) and grads.shape == (n,)
    assert np.isfinite(loss).all() and np.isfinite(params).all() and np.isfinite(grads).all()
    assert float(loss[0]) == pytest.approx(out["final_loss"], abs=1e-6) and np.abs(grads).max() > 0
