"""bench.py's run modes: a plain run measures the headline figure only, ``--full`` adds the sub-lines,
rooflines and CPU baselines, ``--dump-outputs DIR`` writes the last timed step's outputs as .npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_headline_only_and_full_restores_the_rest():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_sub and a.no_roofline and a.no_cpu_baseline
    f = bench.parse_args(["--full"])
    assert f.full and not (f.no_sub or f.no_roofline or f.no_cpu_baseline or f.no_lm)
    n = bench.parse_args(["--full", "--no-lm", "--no-cpu-baseline"])
    assert n.no_lm and n.no_cpu_baseline and not n.no_sub and not n.no_roofline


def test_dump_outputs_small_arrays_whole_large_ones_as_a_fixed_sample(tmp_path):
    import bench
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    share = bench.DUMP_BUDGET_BYTES // 2 // 4
    big = torch.arange(share + 1000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    b = np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(s, np.arange(12, dtype=np.float32))
    # the sample: `share` elements of the array at increasing indices, the same in every run
    assert b.shape == (share,) and np.all(np.diff(b) >= 0) and b[0] >= 0 and b[-1] < share + 1000
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    files = os.listdir(tmp_path / "a")
    assert sorted(files) == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 1000 * 1000


def _bench(args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(dev, tmp_path):
    """Two plain runs with the same arguments: the result line has the headline fields and nothing that
    takes a run of its own, and the dumped metrics / params / grads of the last step agree bit for bit
    (seeded params, batches and dropout; the step is bitwise deterministic)."""
    outs = []
    for d in ("a", "b"):
        o = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert o["steps"] == 3 and o["warmup"] == 1 and o["unit"] == "images/s" and o["higher_is_better"] is True
        assert o["value"] > 0 and o["ms_per_step"] > 0 and o["dtype"].startswith("f32")
        assert abs(o["value"] - 64 / (o["ms_per_step"] * 1e-3)) <= 1e-3 * o["value"]
        assert o["roofline"] is None and o["cpu_baseline"] is None
        assert not any(k in o for k in ("vit_c2_bf16", "vit_c4_soap", "vit_c4_shampoo", "lm124m", "lm420m"))
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = outs
    assert sorted(a) == ["grads.npy", "metrics.npy", "params.npy"]
    for f in a:
        assert a[f].dtype == np.float32 and np.isfinite(a[f]).all()
        assert np.array_equal(a[f], b[f]), f
    assert np.abs(a["grads.npy"]).max() > 0 and a["params.npy"].size == a["grads.npy"].size
    assert abs(float(a["metrics.npy"].reshape(-1)[0]) - o["final_loss"]) < 1e-3
