"""bench.py's plain run and --dump-outputs: a plain run carries no roofline / CPU-baseline leg
(--full turns them on), --steps sets the number of timed steps, and the dump holds the last timed
step's outputs as float32 .npy files, the same from run to run."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_write_outputs_float32_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    big = torch.arange(5000, dtype=torch.float32).view(50, 100)
    arrays = {"small": torch.tensor([1.5, -2.0], dtype=torch.bfloat16), "scalar": torch.tensor(0.25), "big": big}
    bench.write_outputs(str(tmp_path / "a"), arrays)
    bench.write_outputs(str(tmp_path / "b"), arrays)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["big.npy", "scalar.npy", "small.npy"]
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and small.tolist() == [1.5, -2.0]
    assert np.load(tmp_path / "a" / "scalar.npy").dtype == np.float32
    s1, s2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert s1.dtype == np.float32 and s1.shape == (1000,) and np.array_equal(s1, s2)
    # a sample of big's own elements (value == flat index), without repeats, in index order
    assert np.all(np.diff(s1) > 0) and s1.min() >= 0 and s1.max() < 5000


@pytest.mark.gpu
def test_plain_run_and_dump_on_the_gpu(device, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert line["value"] == pytest.approx(line["config"]["global_edges"] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["roofline"] is None and line["cpu_baseline"] is None  # --full only
    names = {p.name for p in out.iterdir()}
    assert {"loss.npy", "logits.npy", "param.convs.0.lin_l.weight.npy", "grad.convs.0.lin_l.weight.npy"} <= names
    total = 0
    for p in out.iterdir():
        a = np.load(p)
        assert a.dtype == np.float32 and np.isfinite(a).all(), p.name
        total += a.nbytes
    assert total <= 64 * 10**6
    assert np.load(out / "logits.npy").shape == (line["config"]["global_nodes"], 2)
    assert np.load(out / "loss.npy") > 0
    assert np.load(out / "param.convs.0.lin_l.weight.npy").shape == (128, 166)
    assert np.abs(np.load(out / "grad.convs.0.lin_l.weight.npy")).max() > 0
