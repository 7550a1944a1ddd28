"""bench.py's plain run and `--dump-outputs`: the options parse, the dump keeps its size
limit with a fixed sample, and (GPU) a plain run times exactly `--steps` frames, leaves what
`--full` measures out of the line and writes the canvas a caller of the timed path receives."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

import bench  # noqa: E402  (the repository root is on sys.path: tests/conftest.py)


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_types_and_limit(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"f64": rng.random((5, 7, 4)), "f32": rng.random(33).astype(np.float32),
              "ints": np.arange(12, dtype=np.int32).reshape(3, 4)}
    written = bench.dump_outputs(tmp_path / "a", arrays)
    assert written == {"f64": 140, "f32": 33, "ints": 12}
    for name, a in arrays.items():
        b = np.load(tmp_path / "a" / (name + ".npy"))
        assert b.dtype == (np.float32 if name == "f32" else np.float64)
        assert b.shape == a.shape and np.array_equal(b, a)
    # over the limit: a fixed sample of the flattened elements, in index order, the same every time
    big = {"x": rng.random(1000), "y": rng.random(10)}
    w1 = bench.dump_outputs(tmp_path / "b", big, max_bytes=1600)
    w2 = bench.dump_outputs(tmp_path / "c", big, max_bytes=1600)
    assert w1 == w2 == {"x": 100, "y": 10}
    x1, x2 = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert x1.tobytes() == x2.tobytes()
    assert sum(np.load(f).nbytes for f in (tmp_path / "b").glob("*.npy")) <= 1600
    idx = np.sort(np.random.default_rng(0).choice(1000, size=100, replace=False))
    assert np.array_equal(x1, big["x"][idx])
    assert np.array_equal(np.load(tmp_path / "b" / "y.npy"), big["y"])


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_canvas(gpu, tmp_path):
    """C1 (200x200x16): the dumped canvas is bit for bit the frame GPURenderer returns for the
    same request (GPU-built tree, forward accumulation, the bench's defaults)."""
    from izpi_amd import _native as N
    from izpi_amd import configs
    from izpi_amd.renderer import GPURenderer
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "2",
                          "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True,
                         timeout=120, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert out.stderr.count("warmup frame") == 1 and "2 of 2 timed frames issued" in out.stderr
    assert line["ms_per_step"] > 0 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(200 * 200 * 16 / line["ms_per_step"] / 1e3, rel=1e-2)
    # what --full measures is left out of a plain run
    assert line["cpu_baseline"] is None and line["roofline"]["achieved"] is None
    d = line["detail"]
    assert d["reference_tree"] is None and d["accumulation_check"] is None and d["host_canvas"] is None
    assert d["dumped_outputs"] == {"canvas": 200 * 200 * 4}
    canvas = np.load(tmp_path / "dump" / "canvas.npy")
    assert canvas.dtype == np.float64 and canvas.shape == (200, 200, 4)
    cfg = configs.configs()["C1"]
    r = GPURenderer(cfg.build(), cfg.width, cfg.height, cfg.spp, max_depth=cfg.max_depth, sampler=cfg.sampler,
                    bvh="gpu", accumulation=N.ACC_FORWARD)
    img = r.render()
    r.close()
    assert canvas.tobytes() == img.tobytes()
