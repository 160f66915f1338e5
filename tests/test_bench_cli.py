"""bench.py's command line: a plain run measures the headline alone, --full adds the CPU baseline
and the nested cfg3 block, --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float_npy(tmp_path):
    t = {"loss": torch.tensor(0.25), "w": torch.arange(12, dtype=torch.bfloat16).reshape(3, 4).float(),
         "count": torch.tensor(3), "d": torch.ones(2, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "o"), t)
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert sorted(got) == ["count", "d", "loss", "w"]
    assert got["loss"].dtype == np.float32 and got["loss"].shape == () and float(got["loss"]) == 0.25
    assert got["count"].dtype == np.float32 and got["d"].dtype == np.float64
    assert np.array_equal(got["w"], np.arange(12, dtype=np.float32).reshape(3, 4))


def test_dump_outputs_samples_beyond_the_limit(tmp_path, monkeypatch):
    """Beyond the limit: a seeded sample, the same elements in every run, small arrays whole."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    big = torch.arange(50_000, dtype=torch.float32)
    small = torch.arange(100, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "big2": big * 2, "small": small})
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 1 << 16
    assert all(np.array_equal(a[f], b[f]) for f in a)
    assert np.array_equal(a["small.npy"], small.numpy())
    assert 1000 < a["big.npy"].size < big.numel() and np.array_equal(a["big2.npy"], 2 * a["big.npy"])
    assert np.all(np.diff(a["big.npy"]) > 0)   # (elements of the flattened array, in order)


def test_make_pool_equals_serial_generation():
    """The forked workers give the meshes make_mesh_graph gives, in seed order."""
    from bgnn import synthetic
    seeds = list(range(100, 116))
    pool = bench.make_pool(6, seeds, False)
    for s, d in zip(seeds, pool):
        ref = synthetic.make_mesh_graph(6, s)
        for k in ("x", "edge_index", "edge_attr", "y"):
            assert torch.equal(getattr(d, k), getattr(ref, k)) and getattr(d, k).dtype == getattr(ref, k).dtype, k


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain run: --steps sets the timed steps, the line has ms_per_step and neither cpu_baseline nor
    cfg3; the dumped loss is the line's final_loss and every file is float32 within the limit."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--store-graphs", "16", "--dump-outputs", str(out)],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "graphs/s" and line["dtype"] == "f32"
    assert line["metric"] == bench.METRIC and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - 16 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    assert "cpu_baseline" not in line and "cfg3" not in line
    files = sorted(os.listdir(out))
    assert "loss.npy" in files and any(f.startswith("param.") for f in files) and any(
        f.startswith("grad.") for f in files)
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    assert all(np.load(out / f).dtype == np.float32 for f in files)
    assert float(np.load(out / "loss.npy")) == pytest.approx(line["final_loss"], rel=1e-6)
    assert all(np.isfinite(np.load(out / f)).all() for f in files if f.startswith("grad."))
