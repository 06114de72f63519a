"""bench.py's plain run and `--dump-outputs`: the CPU part checks the options and the dump format; the GPU part runs a small
plain bench twice and checks the line, the exact step count and that both runs wrote the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_dtypes_shapes_and_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    color = torch.arange(2 * 3 * 8 * 8, dtype=torch.float32).reshape(2, 3, 8, 8)
    radii = torch.arange(2 * 40, dtype=torch.int32).reshape(2, 40)
    nr = [123456789012, 5]
    w = bench.dump_outputs(str(tmp_path / "a"), {"color": color, "radii": radii, "num_rendered": nr})
    assert w == {"color_sample": ((2, 3, 8, 8), 100), "radii": ((2, 40), 80), "num_rendered": ((2,), 2)}
    c = np.load(tmp_path / "a" / "color_sample.npy")
    r = np.load(tmp_path / "a" / "radii.npy")
    n = np.load(tmp_path / "a" / "num_rendered.npy")
    assert c.dtype == np.float32 and r.dtype == np.float32 and n.dtype == np.float64
    pos = np.sort(np.random.default_rng(0).choice(color.numel(), 100, replace=False))
    assert np.array_equal(c, color.reshape(-1).numpy()[pos])
    assert np.array_equal(r, radii.numpy().astype(np.float32)) and n.tolist() == [123456789012.0, 5.0]
    bench.dump_outputs(str(tmp_path / "b"), {"color": color})
    assert np.array_equal(np.load(tmp_path / "b" / "color_sample.npy"), c)


def test_dump_of_the_headline_shapes_stays_under_64_mb():
    a = bench.parse([])
    color = a.views * 3 * a.height * a.width
    radii = a.views * a.gaussians
    total = sum(4 * min(n, bench.DUMP_SAMPLE) for n in (color, radii)) + 8 * a.views
    assert total <= 64 * 2 ** 20


@pytest.mark.gpu
def test_plain_bench_times_exactly_the_steps_and_dumps_the_same_outputs(tmp_path):
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--gaussians", "20000", "--views", "2", "--width", "128",
             "--height", "96"]
    lines = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + ["--dump-outputs", str(tmp_path / run)],
                           cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
        assert line["unit"] == "views/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0 and abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) < 1e-2 * line["value"]
        for key in ("radius_neighbors", "pairs", "extras", "single_view", "roofline"):
            assert key not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["color.npy", "num_rendered.npy", "radii.npy"]
    for name in names:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
    assert np.load(tmp_path / "a" / "color.npy").shape == (2, 3, 96, 128)
    assert np.load(tmp_path / "a" / "radii.npy").shape == (2, 20000)
