"""bench.py's options: `--dump-outputs DIR` (the last timed step's arrays as DIR/<name>.npy) and the plain line without `--full`.
The dump helper is checked on the CPU; the command line end to end on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_ARRAYS = ("color", "radii", "depth", "median", "opacity", "grad_means3D", "grad_shs", "grad_opacities", "grad_scales",
               "grad_rotations", "grad_means2D")


def test_dump_outputs_float32_shapes_and_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    import bench
    big_n = (bench.DUMP_MAX_ELEMS // 5 + 2000) * 5
    g = torch.Generator().manual_seed(3)
    small = torch.randint(0, 50, (7, 5), generator=g, dtype=torch.int32)
    perm = torch.randperm(big_n, generator=g)
    big = perm.to(torch.float32).reshape(-1, 5)                    # distinct values, exact in float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "absent": None})
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (7, 5) and np.array_equal(s, small.numpy().astype(np.float32))
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_MAX_ELEMS,)
    # every sampled value is an element of the array, taken in ascending index order, and the same ones on every run
    inverse = torch.argsort(perm).numpy()
    idx = inverse[b.astype(np.int64)]
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))


def bench_max_elems():
    sys.path.insert(0, ROOT)
    import bench
    return bench.DUMP_MAX_ELEMS


def _run_bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1, r.stdout[-2000:]
    return json.loads(rows[0])


@pytest.mark.gpu
def test_plain_line_and_dump_outputs_identical_from_run_to_run(tmp_path):
    """A plain run: the headline fields, `steps` as asked, none of the `--full` blocks; `--dump-outputs` writes the five outputs and
    six gradients of the last timed step, float32, under 64 MB, and a second run with the same arguments writes the same bits."""
    lines = []
    for d in ("a", "b"):
        lines.append(_run_bench(["--gpus", "1", "--workload", "C2", "--steps", "3", "--warmup", "1", "--settle", "0",
                                 "--dump-outputs", str(tmp_path / d)]))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "Mpixels/s"
    assert line["cpu_baseline"] is None
    for k in ("stage_ms", "roofline", "rotating", "variants", "other_workloads", "reference_hipified_ms"):
        assert k not in line, k
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(STEP_ARRAYS)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += os.path.getsize(tmp_path / "a" / f"{n}.npy")
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "opacity.npy").shape == (1, 800, 800)           # 640 k values: whole
    assert np.load(tmp_path / "a" / "color.npy").shape == (bench_max_elems(),)       # 1.92 M values: the fixed sample
    assert np.abs(np.load(tmp_path / "a" / "grad_means3D.npy")).max() > 0
