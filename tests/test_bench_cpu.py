"""bench.py contract on CPU: ``--gpus 2`` without torchrun re-launches itself
under torch.distributed.run (2 gloo ranks) and prints one JSON line with the
driver's keys; ``--gpus`` must equal WORLD_SIZE; the extras run only with
``--full``; ``--dump-outputs`` writes the last timed step's outputs, the same
in every run."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--device", "cpu", "--rows", "4096", "--features", "16", "--k", "8", "--blobs", "8",
         "--steps", "2", "--warmup", "1", "--no-qpca", "--fit-iters", "3"]


def _run(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=timeout)


def _line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_entry_runs_n_ranks(gpus):
    r = _run(["--gpus", str(gpus), "--full"] + SMALL)
    assert r.returncode == 0, r.stderr[-3000:]
    o = _line(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in o
    assert o["n_gpus"] == gpus and o["steps"] == 2 and o["warmup"] == 1
    assert o["config"]["parallelism"] == f"dp{gpus}" and o["dtype"] == "fp32"
    assert o["value"] > 0 and o["extra"]["rows_per_gpu"] == 4096 // gpus
    fit = [k for k in o["extra"] if k.startswith("fit_wall_s") and not k.endswith("_error")
           and not k.endswith("_n_iter")]
    assert fit, o["extra"]


def test_bench_rejects_world_size_mismatch():
    r = _run(["--gpus", "2"] + SMALL, env_extra={"WORLD_SIZE": "1"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run measures the headline only (no extras) and, with
    ``--dump-outputs``, writes the last step's labels, centres and scalars as
    float32 / float64 ``.npy``; a second run gives the same arrays."""
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = _run(["--gpus", "1", "--dump-outputs", str(d)] + SMALL)
        assert r.returncode == 0, r.stderr[-3000:]
        o = _line(r.stdout)
        assert o["steps"] == 2 and o["ms_per_step"] > 0
        assert o["value"] == pytest.approx(4096 * 2 / (o["ms_per_step"] * 2e-3))
        assert not [k for k in o["extra"] if k.startswith(("fit_wall_s", "qpca", "hard", "ipe"))]
        assert "co_headline" not in o
        assert sorted(os.listdir(d)) == ["centers.npy", "labels.npy", "scalars.npy"]
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = dumps
    assert a["labels"].shape == (4096,) and a["labels"].dtype == np.float32
    assert a["centers"].shape == (8, 16) and a["centers"].dtype == np.float32
    assert a["scalars"].dtype == np.float64 and np.isfinite(a["scalars"]).all()
    assert set(np.unique(a["labels"])) <= set(range(8))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
