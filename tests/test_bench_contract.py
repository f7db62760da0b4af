"""bench.py driver contract on CPU: 2 ranks over gloo via torch.distributed.run, one JSON line from
rank 0 with the fields the driver reads (tiny Gemma-2 geometry on CPU; the GPU run uses the 9B)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_gloo(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs-per-step", "1", "--max-new", "8"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and d["config"]["parallelism"] == "dp2"
    assert d["work"]["cells"] == 2 * 66
    # every timed step all-gathers both ranks' cell records; the SAE thresholds are calibrated identically
    assert d["ranks"]["gathered_rows"] == 2 * 2 * 66
    assert len(d["ranks"]["sae_calib_sha"]) == 2 and len(set(d["ranks"]["sae_calib_sha"])) == 1
    assert d["mem"]["pairs"] == 1 and d["mem"]["auto"] is False


def test_bench_pairs_auto_cpu(tmp_path):
    """``--pairs-per-step auto`` (the default) on CPU: the memory plan is reported and P is its pick."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(OMP_NUM_THREADS="2")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--max-new", "6",
           "--no-config2", "--no-post-forcing"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["mem"]["auto"] is True and d["mem"]["pairs"] >= 1
    assert d["config"]["cells_per_step_per_gpu"] == d["mem"]["pairs"] * 66


SIDES = ("config2", "post_forcing", "lora", "lowrank")


def _run_bench(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(OMP_NUM_THREADS="2")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--max-new", "6"] + list(extra)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_plain_full_and_dump_outputs_cpu(tmp_path):
    """A plain run times its steps only (every side measurement null); ``--full`` adds them.  ``--dump-outputs``
    writes the last timed step's cell records as float .npy arrays, one row per cell, and two runs with the same
    arguments (here: with and without ``--full``) write the same arrays."""
    import numpy as np

    plain = _run_bench(tmp_path, "--dump-outputs", str(tmp_path / "a"))
    assert all(plain[k] is None for k in SIDES)
    assert plain["steps"] == 2 and plain["work"]["cells"] == 2 * plain["config"]["cells_per_step_per_gpu"]
    assert plain["ms_per_step"] > 0 and plain["unit"] == "prompts/s" and plain["higher_is_better"] is True
    # (the post-forcing side takes minutes on CPU: skipped by its own option, as the side sweeps' B = 0 control)
    full = _run_bench(tmp_path, "--full", "--no-post-forcing", "--no-lora-control", "--lowrank-steps", "1",
                      "--side-pairs", "1", "--dump-outputs", str(tmp_path / "b"))
    assert all(full[k] is not None for k in SIDES if k != "post_forcing") and full["post_forcing"] is None
    assert full["lora"]["value"] > 0 and full["lowrank"]["value"] > 0 and full["config2"]["pairs"] == 30
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == sorted(k + ".npy" for k in plain["dumped"]["arrays"])
    n = plain["config"]["cells_per_step_per_gpu"]
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == n and np.isfinite(a).all(), f
        assert a.shape == b.shape and (a == b).all(), f
        total += a.nbytes
    assert 0 < total <= 64e6
    resp = np.load(tmp_path / "a" / "response_ids.npy")
    assert resp.shape == (n, 6) and (resp[:, 0] >= 0).all()


def test_pair_bytes_model():
    """The memory model behind ``--pairs-per-step auto`` at the bench shape: per pair ~1.87 GB of KV / capture /
    pair-KV / lens-sum buffers (round 5 measured 1.83 GB per pair between P = 110 and 120)."""
    sys.path.insert(0, ROOT)
    import bench
    from taboo_brittleness_amd.models.spec import GEMMA2_9B

    per = bench.pair_bytes(GEMMA2_9B, 66, 4, 68, 50)
    assert 1.75e9 < per < 2.0e9, per


def test_bench_self_launch_two_ranks(tmp_path):
    """``bench.py --gpus 2`` with no outer launcher starts the 2 ranks itself (child torch.distributed.run)
    and still prints exactly one JSON line, from rank 0, with the launched world size."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--pairs-per-step", "1", "--max-new", "8"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["ranks"]["world_size"] == 2 and len(d["ranks"]["ms_per_step"]) == 2
